"""Grouped matmul kernels (grouped_gemm.hip) on the GPU: `ops.gemm.grouped_gemm` (forward, and
the data gradient on the transposed weights) and `ops.gemm.grouped_wgrad` against a float64 loop
over the groups on the same bf16 inputs, and `layers.MixtureOfExperts` GPU against CPU.

x, dy and every output are row slices of larger allocations with 256 guard rows on each side and
row strides wider than the rows; everything outside the slices holds a sentinel that must be
unchanged afterwards. Bars (derived, u = 2^-24): bf16 outputs |err| <= 2^-7 |ref| + 2 K u (|x| @ |w|)
— one bf16 ulp of the result plus twice the worst-case fp32 accumulation bound, the MFMA's internal
summation order being unspecified; dw |err| <= 2 max(m_e, 1) u (|x_e|^T @ |dy_e|) + 2^-23 |ref|.
The kernel's row tile is 128: group sizes sit at 127 / 128 / 129."""
import copy
import functools

import pytest
import torch

from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd.ops import gemm as G
from tensorflow_train_distributed_amd.utils import graphs
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

pytestmark = pytest.mark.gpu

GUARD, PAD, SENT = 256, 8, 7.0
U = 2.0 ** -24
EDGE = (0, 1, 127, 128, 129, 0, 257, 0)
_rand = torch.randint(0, 21, (130,), generator=torch.Generator().manual_seed(5))
_rand[::13] = 0
CASES = {
    "edge": (EDGE, 0, 72, 136),
    "edge_tail": (EDGE, 5, 72, 136),
    "one_group": ((130,), 0, 72, 136),
    "last_of_8": ((0,) * 7 + (130,), 0, 72, 136),
    "130_groups": (tuple(_rand.tolist()), 0, 64, 64),
}


def _guarded(rows, width, dtype, pad=PAD):
    """(whole buffer, its [rows, width] slice): the sentinel everywhere, the slice included."""
    whole = torch.full((rows + 2 * GUARD, width + pad), SENT, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + rows, :width]


def _guards_intact(whole, view, what):
    w = whole.clone()
    w[GUARD:GUARD + view.shape[0], :view.shape[1]] = SENT
    assert bool((w == SENT).all()), "%s: written outside its slice" % what


@functools.lru_cache(maxsize=None)
def _case(name):
    """CPU inputs and float64 references of a case, made once and shared (never modified)."""
    sizes, tail, K, N = CASES[name]
    M, E = sum(sizes) + tail, len(sizes)
    g = torch.Generator().manual_seed(11)
    x, dy, w = (torch.randn(s, generator=g).bfloat16() for s in ((M, K), (M, N), (E, K, N)))
    xd, dyd, wd = x.double(), dy.double(), w.double()
    y, dx = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, K, dtype=torch.float64)
    ya, dxa = torch.zeros_like(y), torch.zeros_like(dx)
    dw, dwa = torch.zeros(E, K, N, dtype=torch.float64), torch.zeros(E, K, N, dtype=torch.float64)
    r = 0
    for e, m in enumerate(sizes):
        s = slice(r, r + m)
        y[s], ya[s] = xd[s] @ wd[e], xd[s].abs() @ wd[e].abs()
        dx[s], dxa[s] = dyd[s] @ wd[e].T, dyd[s].abs() @ wd[e].abs().T
        dw[e], dwa[e] = xd[s].T @ dyd[s], 2 * max(m, 1) * U * (xd[s].abs().T @ dyd[s].abs())
        r += m
    offsets = torch.tensor([0] + list(sizes), dtype=torch.int32).cumsum(0, dtype=torch.int32)
    bars = (2.0 ** -7 * y.abs() + 2 * K * U * ya, 2.0 ** -7 * dx.abs() + 2 * N * U * dxa, dwa + 2.0 ** -23 * dw.abs())
    return x, dy, w, offsets, (y, dx, dw), bars


def _run(x, dy, w, offsets):
    """The three kernels on guarded buffers -> ((whole, view) of x, dy, y, dx, dw), after checking the guards."""
    (M, K), N, E = x.shape, dy.shape[1], w.shape[0]
    bufs = [_guarded(M, K, torch.bfloat16), _guarded(M, N, torch.bfloat16), _guarded(M, N, torch.bfloat16),
            _guarded(M, K, torch.bfloat16), _guarded(E * K, N, torch.float32, pad=0)]
    bufs[0][1].copy_(x)
    bufs[1][1].copy_(dy)
    wg, og = w.cuda(), offsets.cuda()
    wt = wg.transpose(1, 2).contiguous()
    G.grouped_gemm(bufs[0][1], wg, og, out=bufs[2][1])
    G.grouped_gemm(bufs[1][1], wt, og, out=bufs[3][1])
    G.grouped_wgrad(bufs[0][1], bufs[1][1], og, out=bufs[4][1].view(E, K, N))
    torch.cuda.synchronize()
    for (whole, view), what in zip(bufs, ("x", "dy", "y", "dx", "dw")):
        _guards_intact(whole, view, what)
    return bufs


@pytest.mark.parametrize("name", list(CASES))
def test_against_float64_loop(name):
    x, dy, w, offsets, refs, bars = _case(name)
    bufs = _run(x, dy, w, offsets)
    tail = CASES[name][1]
    for (_, got), ref, bar, what in zip(bufs[2:], refs, bars, ("y", "dx", "dw")):
        got = got.cpu().double().reshape(ref.shape)
        if tail and what != "dw":
            assert not got[-tail:].any(), "%s: rows of no group must be exactly 0" % what
        ok = (got - ref).abs() <= bar
        ratio = float(((got - ref).abs() / bar.clamp_min(1e-300)).max())
        print("%s %s: worst |err| / bar = %.3f" % (name, what, ratio))
        assert bool(ok.all()), "%s %s: worst |err| / bar = %.3f" % (name, what, ratio)


def test_bad_offsets_stay_inside_the_buffers():
    x, dy, w, offsets, _, _ = _case("edge")
    bad = offsets.clone()
    bad[-1] = x.shape[0] + 40     # past the last row
    bad[4] = bad[3] - 60          # an interior boundary that decreases
    _run(x, dy, w, bad)           # the numbers are anyone's; _run checks the guards


def test_bitwise_repeatable():
    x, dy, w, offsets, _, _ = _case("edge_tail")
    a, b = _run(x, dy, w, offsets), _run(x, dy, w, offsets)
    for (_, p), (_, q) in zip(a[2:], b[2:]):
        assert torch.equal(p, q)


def test_graph_replay_follows_the_offsets_in_device_memory():
    x, dy, w, offsets, _, _ = _case("edge")       # table A: 8 row tiles
    M, E = x.shape[0], w.shape[0]
    table_b = torch.tensor([0, 300, 343] + [M] * (E - 2), dtype=torch.int32)        # 3 + 1 + 3 row tiles
    xg, dyg, wg, og = x.cuda(), dy.cuda(), w.cuda(), offsets.cuda()
    wt = wg.transpose(1, 2).contiguous()
    y, dx = torch.empty_like(dyg), torch.empty_like(xg)
    dw = torch.empty(w.shape, dtype=torch.float32, device="cuda")

    def step():  # one stream, a single chain
        G.grouped_gemm(xg, wg, og, out=y)
        G.grouped_gemm(dyg, wt, og, out=dx)
        G.grouped_wgrad(xg, dyg, og, out=dw)

    captured, _ = graphs.capture(step)
    og.copy_(table_b)
    want = (G.grouped_gemm(xg, wg, og), G.grouped_gemm(dyg, wt, og), G.grouped_wgrad(xg, dyg, og))
    for _ in range(2):
        for o in (y, dx, dw):
            o.fill_(SENT)
        captured.replay()
        torch.cuda.synchronize()
        for got, ref in zip((y, dx, dw), want):
            assert torch.equal(got, ref)


@pytest.mark.parametrize("kind", ["K=68", "misaligned base", "E=0"])
def test_refusals(kind):
    K, E = (68 if kind == "K=68" else 72), (0 if kind == "E=0" else 2)
    x = torch.zeros(16, K + 8, dtype=torch.bfloat16, device="cuda")[:, 4:4 + K] if kind == "misaligned base" else \
        torch.zeros(16, K, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(E, K, 64, dtype=torch.bfloat16, device="cuda")
    dy = torch.zeros(16, 64, dtype=torch.bfloat16, device="cuda")
    off = torch.zeros(E + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(InvalidArgumentError):
        G.grouped_gemm(x, w, off)
    with pytest.raises(InvalidArgumentError):
        G.grouped_wgrad(x, dy, off)


def test_mixture_of_experts_gpu_against_cpu():
    L.reset_naming(seed=0)
    k = 2
    cpu = L.MixtureOfExperts(8, k, 256)
    x = torch.randn(2, 96, 128, generator=torch.Generator().manual_seed(0)).bfloat16().float()
    cpu(x)  # builds the variables
    with torch.no_grad():
        for v in cpu.variables:
            v.copy_(v.bfloat16().float())
    # bf16 differences must not decide the routing: no token's k-th and (k+1)-th logits are close
    top = torch.topk(x.reshape(-1, 128) @ cpu.router_kernel.detach(), k + 1).values
    assert float((top[:, k - 1] - top[:, k]).min()) > 1e-3
    cpu.aux_loss = None  # a graph tensor cannot be deep-copied
    gpu = copy.deepcopy(cpu).to("cuda")
    outs = []
    for layer, xi in ((cpu, x.clone().requires_grad_()), (gpu, x.cuda().requires_grad_())):
        y = layer(xi)
        (y * torch.linspace(-1, 1, 128, device=y.device)).sum().backward()
        outs.append([y.detach().cpu(), xi.grad.cpu()] + [v.grad.cpu() for v in layer.variables])
    torch.testing.assert_close(outs[1][0], outs[0][0], atol=3e-2, rtol=3e-2)
    for got, ref, what in zip(outs[1][1:], outs[0][1:], ("dx", "d router", "d experts_in", "d experts_out")):
        rel = float((got - ref).norm() / ref.norm())
        print("%s: relative L2 %.2e" % (what, rel))
        assert rel < 2e-2, (what, rel)
