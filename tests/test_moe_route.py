"""Mixture-of-experts routing kernels (moe_route.hip) on the GPU through `ops.moe`, against a few
lines of float64 torch written inline, and `layers.MixtureOfExperts` replayed from a graph.

Every output is a slice of a larger allocation filled with a sentinel that must be unchanged
around it. Expert ids, offsets and permutations are compared integer for integer; floating-point
results against float64 with the bars stated beside each constant."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd.ops import _lib
from tensorflow_train_distributed_amd.ops import moe as M
from tensorflow_train_distributed_amd.utils import graphs
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, -7
U32, UBF = 2.0 ** -24, 2.0 ** -8   # unit roundoffs of fp32 and bf16
# The float64 statements of _route_ref run in float32 on the CPU differ from float64 by at most
# 2.04e-7 in probs and gate over every case below (both are <= 1); 4 times that for another exp.
ROUTE_BAR = 4 * 2.04e-7
# The float64 autograd of _route_grad run in float32 on the CPU: the worst |error| of a row over the
# row's sum_e p_e |dL/dp_e| (the terms dlogits cancels; not below 2^-126, where fp32 underflows) is
# 2.92e-6 over every case and gradient mode below; 4 times that.
ROUTE_BWD_BAR = 4 * 2.92e-6

ROUTE_CASES = [(1, 1, 1), (3, 2, 2), (65, 8, 2), (130, 64, 8), (67, 65, 4), (33, 256, 8),
               (37, 9, 3), (37, 17, 4), (37, 33, 5), (35, 129, 8), (33, "max", "max")]


def _guarded(rows, width, dtype, pad=0):
    """(whole buffer, its [rows, width] slice) full of the sentinel; width None: a 1-D slice."""
    whole = torch.full((rows + 2 * GUARD, (width or 1) + pad), SENT, dtype=dtype, device="cuda")
    view = whole[GUARD:GUARD + rows, :width or 1]
    return whole, (view if width else view[:, 0])


def _intact(whole, view, what):
    w = whole.clone()
    w[GUARD:GUARD + view.shape[0], :(view.shape[1] if view.dim() == 2 else 1)] = SENT
    assert bool((w == SENT).all()), "%s: written outside its slice" % what


def _route_ref(logits, expert, dtype):
    p = torch.softmax(logits.to(dtype), -1)
    g = p.gather(1, expert)
    return p, g / g.sum(-1, keepdim=True)


@functools.lru_cache(maxsize=None)
def _route_case(T, E, k):
    """Logits with the planted rows, the float64 selection (lowest index on ties) and references."""
    x = 4 * torch.randn(T, E, generator=torch.Generator().manual_seed(T * 1000 + E))
    x[0] = 0.5                                                  # all equal
    for t in range(1, T, 5):                                    # exact ties across the k / k+1 boundary
        if E > k:
            top = torch.topk(x[t], k + 1).indices
            x[t, top[k]] = x[t, top[k - 1]]
    if T > 2:
        x[2, 0], x[2, -1] = 88.0, -88.0
    if T > 3 and E - k > 1:
        x[3, torch.randperm(E, generator=torch.Generator().manual_seed(1))[:min(3, E - k - 1)]] = -float("inf")
    expert = torch.sort(x.double(), dim=-1, descending=True, stable=True).indices[:, :k]
    return x, expert, _route_ref(x, expert, torch.float64)


def _route_grad(x, expert, dgate, dprobs, dtype):
    """(dlogits, the row's sum_e p_e |dL/dp_e|: the size of the terms dlogits cancels) by autograd."""
    xd = x.clone().to(dtype).requires_grad_()
    p, g = _route_ref(xd, expert, dtype)
    p.retain_grad()
    loss = (0 if dgate is None else (g * dgate.to(dtype)).sum()) + (0 if dprobs is None else (p * dprobs.to(dtype)).sum())
    loss.backward()
    return xd.grad.double(), (p.detach() * p.grad.abs()).sum(1).double()


def _route_shape(T, E, k):
    return T, (M.max_experts() if E == "max" else E), (M.max_topk() if k == "max" else k)


def _run_topk(x, k):
    T, E = x.shape
    bufs = [_guarded(T, E, torch.float32), _guarded(T, k, torch.int32), _guarded(T, k, torch.float32)]
    xg = torch.full((T + 2, E + 3), 9.0, device="cuda")[1:T + 1, :E]  # strided rows
    xg.copy_(x)
    M.topk_route(xg, k, out=tuple(v for _, v in bufs))
    torch.cuda.synchronize()
    for (whole, view), what in zip(bufs, ("probs", "expert", "gate")):
        _intact(whole, view, what)
    return [v for _, v in bufs]


@pytest.mark.parametrize("shape", ROUTE_CASES, ids=str)
def test_topk_against_float64(shape):
    T, E, k = _route_shape(*shape)
    x, expert, (p64, g64) = _route_case(T, E, k)
    probs, got, gate = _run_topk(x, k)
    assert torch.equal(got.cpu().long(), expert)
    for what, a, ref in (("probs", probs, p64), ("gate", gate, g64)):
        err = float((a.cpu().double() - ref).abs().max())
        print("%s %s: worst |err| %.3g, bar %.3g" % (shape, what, err, ROUTE_BAR))
        assert err <= ROUTE_BAR, (what, err)


@pytest.mark.parametrize("mode", ["both", "dgate", "dprobs"])
@pytest.mark.parametrize("shape", ROUTE_CASES, ids=str)
def test_topk_bwd_against_float64_autograd(shape, mode):
    T, E, k = _route_shape(*shape)
    x = _route_case(T, E, k)[0]
    probs, expert, gate = (v.contiguous() for v in _run_topk(x, k))
    g = torch.Generator().manual_seed(3)
    dgate = torch.randn(T, k, generator=g) if mode != "dprobs" else None
    dprobs = torch.randn(T, E, generator=g) if mode != "dgate" else None
    whole, out = _guarded(T, E, torch.float32)
    M.topk_route_bwd(probs, expert, gate, None if dgate is None else dgate.cuda(),
                     None if dprobs is None else dprobs.cuda(), out=out)
    torch.cuda.synchronize()
    _intact(whole, out, "dlogits")
    ref, scale = _route_grad(x, expert.cpu().long(), dgate, dprobs, torch.float64)
    ratio = float(((out.cpu().double() - ref).abs().amax(1) / scale.clamp_min(2.0 ** -126)).max())
    print("%s %s: worst row |err| / sum p |dp| %.3g, bar %.3g" % (shape, mode, ratio, ROUTE_BWD_BAR))
    assert ratio <= ROUTE_BWD_BAR


def _sort_ref(ids, E):
    key = torch.where((ids >= 0) & (ids < E), ids, torch.full_like(ids, E)).long()
    offsets = F.pad(torch.bincount(key, minlength=E + 1)[:E].cumsum(0), (1, 0))
    order = torch.argsort(key, stable=True)
    return offsets, order, torch.argsort(order)


@pytest.mark.parametrize("E", [1, 8, 65, 1024])
@pytest.mark.parametrize("S", [(0, 1), (0, 63), (0, 64), (0, 65), (1, -1), (1, 0), (1, 1), (3, 17)], ids=str)
def test_sort_exact(S, E):
    S = S[0] * M.sort_chunk() + S[1]                            # (chunks, slots past them)
    g = torch.Generator().manual_seed(S + E)
    planted = torch.randint(0, E, (S,), generator=g, dtype=torch.int32)
    planted[torch.randperm(S, generator=g)[:S // 3 + 1]] = torch.tensor([-1, E, 2 ** 31 - 1], dtype=torch.int32)[
        torch.randint(0, 3, (S // 3 + 1,), generator=g)]
    for kind, ids in (("random", torch.randint(0, E, (S,), generator=g, dtype=torch.int32)),
                      ("one expert", torch.full((S,), E // 2, dtype=torch.int32)),
                      ("last expert", torch.full((S,), E - 1, dtype=torch.int32)), ("planted", planted)):
        runs = []
        for _ in range(2):
            ws_n = M.sort_workspace(S, E, "cuda").numel()
            bufs = [_guarded(E + 1, None, torch.int32), _guarded(S, None, torch.int32), _guarded(S, None, torch.int32),
                    _guarded(ws_n, None, torch.int32)]
            M.sort_by_expert(ids.cuda(), E, out=tuple(v for _, v in bufs[:3]), workspace=bufs[3][1])
            torch.cuda.synchronize()
            for (whole, view), what in zip(bufs, ("offsets", "order", "inv", "workspace")):
                _intact(whole, view, kind + " " + what)
            runs.append([v.cpu() for _, v in bufs[:3]])
        for got, ref, what in zip(runs[0], _sort_ref(ids, E), ("offsets", "order", "inv")):
            assert torch.equal(got.long(), ref), (kind, what)
        assert torch.equal(runs[0][2][runs[0][1].long()], torch.arange(S, dtype=torch.int32))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), kind + ": two runs differ"


def _rows(rows, D, dtype, gen=None):
    """A guarded [rows, D] slice with a row stride of D + 8; random (bf16-exact) values if gen."""
    whole, view = _guarded(rows, D, dtype, pad=8)
    if gen is not None:
        view.copy_(torch.randn(rows, D, generator=gen).bfloat16())
    return whole, view


def _close(got, ref, abs_sum, n, u_out, what):
    """|err| <= one rounding of the output type + (n + 2) fp32 roundoffs of the sum of |terms|."""
    bar = u_out * ref.abs() + (n + 2) * U32 * abs_sum
    ratio = float(((got.cpu().double() - ref).abs() / bar.clamp_min(1e-300)).max())
    print("%s: worst |err| / bar = %.3f" % (what, ratio))
    assert ratio <= 1.0, what


@pytest.mark.parametrize("types", [(torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32),
                                   (torch.float32, torch.bfloat16)], ids=str)
@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("D,side", [(8, "lo"), (136, "lo"), (1032, "lo"), (1032, "hi")])
def test_gather_combine(D, side, k, types):
    sdt, odt = types
    trip = _lib.query("ttdk_moe_row_max_threads") // (D // 8)   # rows one grid-stride trip covers
    T = 37 if D < 1032 else (trip // k if side == "lo" else -(-(trip + 2) // k))
    R, E, u_out = T * k, 5, (UBF if odt == torch.bfloat16 else U32)
    g = torch.Generator().manual_seed(D + k)
    ids = torch.randint(0, E, (T, k), generator=g, dtype=torch.int32)
    ids.view(-1)[torch.randperm(R, generator=g)[:R // 7 + 1]] = torch.tensor([-1, E], dtype=torch.int32)[
        torch.randint(0, 2, (R // 7 + 1,), generator=g)]        # slots of no group
    offsets, order, inv = M.sort_by_expert(ids.cuda(), E)
    assert all(torch.equal(a.cpu().long(), b) for a, b in zip((offsets, order, inv), _sort_ref(ids.view(-1), E)))
    valid = ((ids >= 0) & (ids < E)).double()
    (sw, src), (hw, h), (cw, hs) = _rows(T, D, sdt, g), _rows(R, D, odt, g), _rows(R, D, sdt, g)
    gate = torch.rand(T, k, generator=g) + 0.25
    src64, h64, hs64, o, i = src.cpu().double(), h.cpu().double(), hs.cpu().double(), order.cpu().long(), inv.cpu().long()
    # dispatch: a pure gather is bit for bit, the cast included
    (ow, out) = _rows(R, D, odt)
    M.gather_rows(src, order, k, out=out)
    assert torch.equal(out, src[o.cuda() // k].to(odt))
    # the combine's backward: dh = gate[slot] * dy[slot // k] and dgate[slot] = dot(h[row], dy[slot // k])
    (dw, dh) = _rows(R, D, odt)
    _, dgate = M.gather_rows(src, order, k, scale=gate.cuda(), h=h, out=dh)
    ref = gate.double().view(-1)[o, None] * src64[o // k]
    _close(dh, ref, ref.abs(), 1, u_out, "dh")
    _close(dgate, (h64[i] * src64.repeat_interleave(k, 0)).sum(1), (h64[i] * src64.repeat_interleave(k, 0)).abs().sum(1),
           D, U32, "dgate")
    # a scaled gather without the dot; idx entries outside the slots give zero rows
    bad, (gw, gs) = order.clone(), _rows(R, D, odt)
    bad[0], bad[1], ref[:2] = -1, R, 0
    M.gather_rows(src, bad, k, scale=gate.cuda(), out=gs)
    _close(gs, ref, ref.abs(), 1, u_out, "scaled gather")
    assert not gs[:2].any()
    # combine, with the rows of no group zeroed as the grouped kernels leave them; an inv entry
    # outside the rows (slot 0 here) adds nothing
    hs[int(offsets[E]):] = 0
    bad = inv.clone()
    bad[0], valid.view(-1)[0] = R, 0
    for w in (gate, None):
        (yw, y) = _rows(T, D, odt)
        M.combine_rows(hs, bad, k, w=None if w is None else w.cuda(), out=y)
        terms = (valid if w is None else valid * w.double())[:, :, None] * hs64[i].view(T, k, D)
        _close(y, terms.sum(1), terms.abs().sum(1), k, u_out, "combine" + (" weighted" if w is not None else ""))
        _intact(yw, y, "y")
    torch.cuda.synchronize()
    for whole, view, what in ((sw, src, "src"), (hw, h, "h"), (cw, hs, "hs"), (ow, out, "out"), (dw, dh, "dh"),
                              (gw, gs, "gs")):
        _intact(whole, view, what)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_gather_slots_past_2_24_times_k(k):
    """idx // k is exact over the whole admitted range: a reciprocal with a 40-bit shift overflows
    64 bits from slot 2^24 * k on and would fetch other, in-bounds rows."""
    n = 2 ** 24 + 8
    row = torch.arange(n, device="cuda")
    src = torch.zeros(n, 8, device="cuda")
    src[:, 0], src[:, 1] = row % 4096, row // 4096              # the row number, exactly, in two floats
    idx = torch.tensor([0, 2 ** 24 - 1, 2 ** 24, 2 ** 24 * k + 3, n * k - 1], dtype=torch.int32, device="cuda")
    assert torch.equal(M.gather_rows(src, idx, k), src[idx.long() // k])


def _refused():
    f32, bf = torch.float32, torch.bfloat16
    z = lambda *s, dt=f32, dev="cuda": torch.zeros(*s, dtype=dt, device=dev)
    idx = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    return {
        "E above the limit": lambda: M.topk_route(z(4, M.max_experts() + 1), 2),
        "k above the limit": lambda: M.topk_route(z(4, 64), M.max_topk() + 1),
        "k > E": lambda: M.topk_route(z(4, 3), 4),
        "sort E above the limit": lambda: M.sort_by_expert(idx(8), _lib.query("ttdk_grouped_gemm_max_groups") + 1),
        "D = 12": lambda: M.gather_rows(z(4, 12, dt=bf), idx(4)),
        "misaligned base": lambda: M.gather_rows(z(4, 24, dt=bf)[:, 4:20], idx(4)),
        "misaligned combine": lambda: M.combine_rows(z(4, 24)[:, 2:18], idx(4), 1),
        "bf16 logits": lambda: M.topk_route(z(4, 8, dt=bf), 2),
        "int64 ids": lambda: M.sort_by_expert(torch.zeros(8, dtype=torch.int64, device="cuda"), 4),
        "fp16 rows": lambda: M.combine_rows(z(4, 16, dt=torch.float16), idx(4), 1),
        "int64 idx": lambda: M.gather_rows(z(4, 16), torch.zeros(4, dtype=torch.int64, device="cuda")),
        "logits on the CPU": lambda: M.topk_route(z(4, 8, dev="cpu"), 2),
        "idx on the CPU": lambda: M.gather_rows(z(4, 16), torch.zeros(4, dtype=torch.int32)),
        "dgate on the CPU": lambda: M.topk_route_bwd(z(4, 8), idx(8).view(4, 2), z(4, 2), z(4, 2, dev="cpu")),
    }


@pytest.mark.parametrize("kind", ["E above the limit", "k above the limit", "k > E", "sort E above the limit", "D = 12",
                                  "misaligned base", "misaligned combine", "bf16 logits", "int64 ids", "fp16 rows",
                                  "int64 idx", "logits on the CPU", "idx on the CPU", "dgate on the CPU"])
def test_refusals(kind, monkeypatch):
    call = _refused()[kind]

    def launched(name, *a):
        raise AssertionError("%s was launched" % name)

    monkeypatch.setattr(_lib, "call", launched)
    with pytest.raises(InvalidArgumentError):
        call()


def test_layer_graph_replay_follows_the_routing():
    L.reset_naming(seed=0)
    layer = L.MixtureOfExperts(8, 2, 256)
    g = torch.Generator().manual_seed(0)
    xa, xb = (torch.randn(2, 96, 128, generator=g).bfloat16().float() for _ in range(2))
    layer(xa)  # builds the variables
    layer.aux_loss = None
    layer = layer.to("cuda")
    sizes = [torch.topk(x.reshape(-1, 128) @ layer.router_kernel.detach().cpu(), 2).indices.flatten().bincount(minlength=8)
             for x in (xa, xb)]
    assert not torch.equal(*sizes)
    x = xa.cuda().requires_grad_()
    weight = torch.linspace(-1, 1, 128, device="cuda")

    def step():
        for v in [x] + list(layer.variables):
            v.grad = None
        y = layer(x)
        (y * weight).sum().backward()
        return [y.detach(), x.grad] + [v.grad for v in layer.variables]

    captured, outs = graphs.capture(step)
    with torch.no_grad():
        x.copy_(xb)
    for _ in range(2):
        captured.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        for a, b in zip(got, step()):
            assert torch.equal(a, b)
