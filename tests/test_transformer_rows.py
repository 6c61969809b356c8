"""The row kernels of csrc/kernels/transformer.hip (LayerNorm forward / backward and its
colreduce, the embedding gather and its three gradients, row gather / scatter, the valid-label
count, the vocabulary cross-entropy, dact, tanh_) against the float64 statements of
tests/transformer_oracle.py, at the shapes where each kernel takes another path.

Every comparison is element-wise: |got - want| <= half a bf16 ulp of want (bf16 outputs only: the
store) + bar * scale, with the scale of each figure and its bar in transformer_oracle.BARS. A bar
is 16 x the largest value the same figure takes when the oracle itself runs in float32
(tests/test_transformer_oracle_cpu.py), never less than 16 x 2^-24. Operations that are exact are
compared exactly. Outputs sit between guard rows of a fixed byte pattern that must survive.

LayerNorm: the kernels round s to bf16 before they take its statistics, so s is checked first
(within one bf16 ulp of the reference plus the fp32 bar; exactly where the fp32 sum is exact),
then mean and rstd against the statistics of that s, then y and the backward from that s and
those fp32 statistics, which are what the backward kernel is handed.

Largest figure of any case on an MI355X, beside its bar (fp32: the float32 oracle):

  figure        MI355X     fp32      bar
  ln_s          4.5e-8     1.3e-7    3e-6
  ln_mean       2.5e-8     2.5e-8    1e-6
  ln_rstd       5.0e-7     1.7e-7    3e-6
  ln_y          1.5e-7     2.7e-7    5e-6
  ln_ds         4.8e-8     2.4e-7    4e-6
  ln_dx         5.9e-8     2.4e-7    4e-6
  ln_dgamma     1.6e-7     1.6e-7    3e-6
  ln_dbeta      7.0e-8     6.2e-8    1e-6
  emb_s         8.8e-9     7.9e-8    2e-6
  emb_dword     1.2e-7     8.8e-8    2e-6   (atomics: the last digit moves from run to run)
  emb_dpos      6.8e-8     7.8e-8    2e-6
  emb_dtype     1.5e-8     1.7e-8    1e-6   (parent commit: 0.07 .. 0.24 at H = 768 and 1536)
  scatter       4e-19      0         1e-6
  count         3.5e-8     5.0e-8    1e-6
  xent_grad     2e-13      1.0e-7    2e-6   (all of the error is inside the store's half ulp)
  xent_loss     6.7e-8     4.8e-8    1e-6
  xent_correct  0          0         1e-6
  dact          4.4e-7     5.0e-7    9e-6
  tanh          0          3.0e-8    1e-6

The half ulp is that of `want` itself, 2^(e-9) for |want| in [2^(e-1), 2^e): between 2^-9 and 2^-8
of |want|. A flat 2^-9 * |want| cannot hold for a correctly rounded store (want = 1.003 stores as
1.0, an error of 2^-8.4 * |want|).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import transformer_oracle as O
from tensorflow_train_distributed_amd.ops import _lib
from tensorflow_train_distributed_amd.ops import transformer as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))
PATTERN = 0x5A


class Guarded:
    """A tensor `t` of `shape` with O.GUARD rows (elements of a 1-D shape) of the byte PATTERN on
    either side in one allocation; `t` starts out as the pattern too, so what a kernel leaves
    unwritten shows."""

    def __init__(self, shape, dtype, init=None):
        shape = tuple(shape)
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape)) * item
        self.g = O.GUARD * (int(np.prod(shape[1:])) if len(shape) > 1 else 1) * item
        self.raw = torch.full((2 * self.g + n,), PATTERN, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.g:self.g + n].view(dtype).view(shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.raw[:self.g] == PATTERN).all()) and bool((self.raw[self.g + self.t.numel()
                                                                             * self.t.element_size():] == PATTERN).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _digest(t):
    return hashlib.sha256(_bits(t).cpu().numpy().tobytes()).hexdigest()


def _dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


# ------------------------------------------------------------------ LayerNorm
def _ln_case(mode, H, rows, want_dx=True, accumulate=False, adjacent=False):
    """Forward and backward of one case with every check that holds for all of them; returns the
    outputs (ds, dx, dgamma, dbeta, ...) for the tests that compare two runs."""
    residual, p_in, p_out, eps = O.LN_MODES[mode]
    inp = _dev(O.ln_inputs(mode, H, rows))
    kin, kout = O.ln_masks(mode, H, rows, DEV)
    x0 = inp["x"].clone()
    rng = T.RngState(O.SEED, DEV)
    assert rng.host() == (O.SEED, O.STEP)
    drop = dict(p_in=p_in, site_in=O.SITE_IN, p_out=p_out, site_out=O.SITE_OUT, rng=rng)
    y, mean, rstd = Guarded((rows, H), BF16), Guarded((rows,), F32), Guarded((rows,), F32)
    writes_s = residual or p_in > 0
    sbuf = Guarded((rows, H), BF16) if writes_s else None
    _, s, _, _ = T.layernorm_fwd(inp["x"], inp["gamma"], inp["beta"], res=inp["res"], eps=eps, out=y.t,
                                 s_out=sbuf.t if writes_s else None, mean=mean.t, rstd=rstd.t, **drop)
    assert torch.equal(inp["x"], x0)
    if writes_s:
        assert s.data_ptr() == sbuf.t.data_ptr() and sbuf.intact()
    else:
        assert s.data_ptr() == inp["x"].data_ptr()  # no residual, no input dropout: s is x itself
    s_ref = O.ln_s(inp["x"], inp["res"], kin, p_in)
    fig_s = {"ln_s": O.figure(s, s_ref, O.ln_s_scale(inp["x"], inp["res"], p_in), bf16_store=True, ulps=1.0)}
    print("layernorm", mode, H, rows, fig_s)
    O.check(fig_s, (mode, H, rows))
    if p_in == 0:
        fp32_sum = inp["x"].float() + inp["res"].float() if residual else inp["x"].float()
        exact = fp32_sum.to(F64) == s_ref
        assert float(exact.float().mean()) > 0.5
        assert torch.equal(s[exact], fp32_sum.to(BF16)[exact])
    assert y.intact() and mean.intact() and rstd.intact()

    dg0 = db0 = None
    if accumulate:
        dg0 = torch.randn(H, generator=O._gen(H, 99)).to(DEV)
        db0 = torch.randn(H, generator=O._gen(H, 98)).to(DEV)
    if adjacent:
        both = Guarded((2, H), F32)
        dgb, dbb = both.t[0], both.t[1]
        assert dbb.data_ptr() == dgb.data_ptr() + 4 * H
        guards = [both]
    else:
        gg, gb = Guarded((H,), F32), Guarded((H,), F32)
        dgb, dbb = gg.t, gb.t
        guards = [gg, gb]
    if accumulate:
        dgb.copy_(dg0)
        dbb.copy_(db0)
    ds, dx = Guarded((rows, H), BF16), Guarded((rows, H), BF16)
    ds_t, dx_t = T.layernorm_bwd(inp["dy"], s, mean.t, rstd.t, inp["gamma"], dgb, dbb, ds_out=ds.t, want_dx=want_dx,
                                 accumulate=accumulate, dx_out=dx.t if want_dx else None, **drop)
    torch.cuda.synchronize()
    assert ds_t.data_ptr() == ds.t.data_ptr() and (dx_t is None) == (not want_dx)
    assert ds.intact() and dx.intact() and all(g.intact() for g in guards)
    if not want_dx:
        assert bool((dx.raw == PATTERN).all())

    stats = (mean.t, rstd.t)
    ref = O.ln_reference(mode, inp, kin, kout, s, stats, dg0, db0)
    scales = O.ln_scales(mode, inp, kout, s, ref, stats, dg0, db0)
    got = {"mean": mean.t, "rstd": rstd.t, "y": y.t, "ds": ds.t, "dx": dx.t if want_dx else None,
           "dgamma": dgb, "dbeta": dbb}
    figs = O.ln_figures(got, ref, scales)
    print("layernorm", mode, H, rows, {k: "%.2e" % v for k, v in figs.items()})
    O.check(figs, (mode, H, rows))
    if want_dx and p_in == 0:
        assert _same_bits(dx.t, ds.t)
    if rows >= 77 and p_out == 0:
        # a constant row: s - mean is exactly 0, so y is beta rounded to bf16
        assert torch.equal(y.t[O.ROW_CONST], inp["beta"].to(BF16))
    return {"ds": ds.t, "dx": dx.t if want_dx else None, "dgamma": dgb.clone(), "dbeta": dbb.clone()}


@pytest.mark.parametrize("mode,H,rows", O.LN_GRID + O.LN_ENGINE + O.LN_EXTRA)
def test_layernorm_fwd_bwd(mode, H, rows):
    """rows = 1; 77 (an odd last block, several trips per wave at the 4-wave widths); 4097 (the
    256-block cap, 17 rows per block, blocks 241..255 own no row). Modes: transformer_oracle.LN_MODES."""
    _ln_case(mode, H, rows)


def test_layernorm_bwd_without_dx():
    _ln_case("both", 1024, 77, want_dx=False)


def test_layernorm_bwd_accumulates_onto_old_gradients():
    _ln_case("layer", 1024, 77, accumulate=True)


@pytest.mark.parametrize("rows", [77, 4097])
def test_layernorm_bwd_adjacent_and_separate_gradients_bit_equal(rows):
    """dgamma and dbeta as the two halves of one buffer (one colreduce launch over 2H columns, the
    flat gradient store's layout) and as separate tensors (two launches)."""
    a = _ln_case("both", 1024, rows, adjacent=True)
    b = _ln_case("both", 1024, rows, adjacent=False)
    for k in ("ds", "dx", "dgamma", "dbeta"):
        assert _same_bits(a[k], b[k]), k


def prefetch0_child():
    """Runs in the child of the test below, TTD_LN_BWD_PREFETCH=0 in its environment."""
    assert os.environ.get("TTD_LN_BWD_PREFETCH") == "0"
    for mode, H, rows in O.LN_PREFETCH0:
        out = _ln_case(mode, H, rows)
        print("DIGEST", rows, _digest(out["ds"]), _digest(out["dx"]), _digest(out["dgamma"]), _digest(out["dbeta"]))


def test_layernorm_bwd_two_rows_in_flight_kernel():
    """TTD_LN_BWD_PREFETCH=0 selects ln_bwd_kernel<2, 8, 2> at H = 1024 (two rows in flight per
    wave, wave_sum4); the variable is read once per process, hence the child. rows = 9 leaves wave
    1's second row missing. Same bars (checked in the child); ds / dx / dgamma / dbeta bit-equal to
    the default kernel's: the per-row arithmetic and the order of every sum are the same."""
    assert os.environ.get("TTD_LN_BWD_PREFETCH", "1") != "0"
    default = {}
    for mode, H, rows in O.LN_PREFETCH0:
        out = _ln_case(mode, H, rows)
        default[rows] = [_digest(out[k]) for k in ("ds", "dx", "dgamma", "dbeta")]
    env = dict(os.environ, TTD_LN_BWD_PREFETCH="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_transformer_rows as t; t.prefetch0_child()" % (
        os.path.dirname(HERE), HERE)
    p = subprocess.run([sys.executable, "-c", code], cwd=HERE, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=180)
    print(p.stdout[-4000:])
    assert p.returncode == 0, p.stdout[-4000:]
    child = {int(l.split()[1]): l.split()[2:] for l in p.stdout.splitlines() if l.startswith("DIGEST")}
    assert sorted(child) == sorted(default)
    for rows in default:
        assert child[rows][:2] == default[rows][:2], ("ds / dx differ from the default kernel", rows)
        assert child[rows][2:] == default[rows][2:], ("dgamma / dbeta differ from the default kernel", rows)


# ------------------------------------------------------------------ vocabulary cross-entropy
GSC, MSC = 0.37, 0.25
SUMS0 = (3.0, 5.0)


def _xent_run(z, V, labels, dl, mscale=True, sums=True):
    s = torch.tensor(SUMS0, device=DEV) if sums else None
    T.xent_vocab(z, V, labels, torch.tensor([GSC], device=DEV), dlogits=dl, sums=s,
                 mscale=torch.tensor([MSC], device=DEV) if mscale else None)
    torch.cuda.synchronize()
    return s


def _xent_sums_figures(z, V, labels, sums, msc):
    _, _, _, want = O.xent(z, V, labels, GSC, msc)
    sl, sc = O.xent_scales(z, V, labels, msc)
    return {"xent_loss": abs(float(sums[0]) - SUMS0[0] - want[0]) / (sl + SUMS0[0]),
            "xent_correct": abs(float(sums[1]) - SUMS0[1] - want[1]) / (sc + SUMS0[1])}


@pytest.mark.parametrize("V,ld", O.XENT_CASES)
def test_xent_vocab(V, ld):
    """(5, 8): one thread, all tail; (1000, 1024): one trip; (2048, 2048): no padding, no tail;
    (2049, 2056): a second trip that is a one-element tail; (30522, 30528): BERT's vocabulary, 15
    trips and a two-element tail. Rows: transformer_oracle.xent_inputs."""
    z, labels = (t.to(DEV) for t in O.xent_inputs(V, ld))
    z0 = z.clone()
    _, _, grad, _ = O.xent(z, V, labels, GSC, MSC)
    # the gradient into a buffer of its own
    dl = Guarded((O.XENT_ROWS, ld), BF16)
    sums = _xent_run(z, V, labels, dl.t)
    assert torch.equal(z, z0) and dl.intact()
    figs = {"xent_grad": O.figure(dl.t, grad, GSC, bf16_store=True)}
    figs.update(_xent_sums_figures(z, V, labels, sums, MSC))
    print("xent", V, ld, {k: "%.2e" % v for k, v in figs.items()})
    O.check(figs, (V, ld))
    assert bool((dl.t[:, V:].float() == 0).all()), "padding columns"
    assert bool((dl.t[labels < 0].float() == 0).all()), "ignored rows"
    # in place: the same bits
    zi = Guarded((O.XENT_ROWS, ld), BF16, init=z)
    sums_i = _xent_run(zi.t, V, labels, zi.t)
    assert zi.intact() and _same_bits(zi.t, dl.t)
    O.check(_xent_sums_figures(z, V, labels, sums_i, MSC), (V, ld, "in place"))
    # no gradient wanted: the sums alone
    sums_n = _xent_run(z, V, labels, None)
    assert torch.equal(z, z0)
    O.check(_xent_sums_figures(z, V, labels, sums_n, MSC), (V, ld, "no dlogits"))
    # no metric scale: 1
    dl2 = Guarded((O.XENT_ROWS, ld), BF16)
    sums_1 = _xent_run(z, V, labels, dl2.t, mscale=False)
    O.check(_xent_sums_figures(z, V, labels, sums_1, 1.0), (V, ld, "no mscale"))
    assert _same_bits(dl2.t, dl.t)
    # no sums wanted
    dl3 = Guarded((O.XENT_ROWS, ld), BF16)
    _xent_run(z, V, labels, dl3.t, sums=False)
    assert _same_bits(dl3.t, dl.t) and dl3.intact()


@pytest.mark.parametrize("V,ld", [(5, 8), (30522, 30528)])
def test_xent_vocab_every_label_ignored(V, ld):
    z, labels = (t.to(DEV) for t in O.xent_inputs(V, ld))
    labels.fill_(-1)
    out = torch.full((4,), -7.0, device=DEV)
    T.count_valid(labels, 3.0, out)
    assert out.tolist() == [3.0, -7.0, -7.0, -7.0]  # the count is clamped to 1
    dl = Guarded((O.XENT_ROWS, ld), BF16)
    sums = _xent_run(z, V, labels, dl.t)
    assert sums.tolist() == list(SUMS0)
    assert bool((dl.t.float() == 0).all()) and dl.intact()


@pytest.mark.parametrize("n", O.COUNT_N)
def test_count_valid_both_forms(n):
    labels = torch.randint(0, 1000, (n,), generator=O._gen(n, 17), dtype=torch.int32)
    labels[2::3] = -1
    labels[1::7] = -100
    labels = labels.to(DEV)
    one = torch.full((4,), -7.0, device=DEV)
    two = torch.full((4,), -7.0, device=DEV)
    T.count_valid(labels, 3.0, one)
    T.count_valid2(labels, 3.0, two)
    assert one[1:].tolist() == [-7.0] * 3 and two[2:].tolist() == [-7.0] * 2
    (w1,) = O.count_valid(labels, 3.0)
    w2 = O.count_valid(labels, 3.0, both=True)
    figs = {"count": max(abs(float(one[0]) - w1) / w1, abs(float(two[0]) - w2[0]) / w2[0],
                         abs(float(two[1]) - w2[1]) / w2[1])}
    print("count", n, figs)
    O.check(figs, n)


# ------------------------------------------------------------------ embeddings
#             H, T, token types, pos_beta, type gradient wanted, one id for every row
EMBED_CASES = [(H, 2, True, 0, True, False) for H in O.EMBED_H] + [
    (768, 1, True, 1, True, False), (768, 4, True, 0, True, False), (1536, 4, True, 1, True, False),
    (1536, 1, False, 0, True, False), (1024, 2, False, 0, True, False), (512, 2, True, 1, False, False),
    (1536, 2, True, 0, True, True), (128, 4, True, 1, True, True)]


@pytest.mark.parametrize("H,T_,with_tt,pos_beta,want_type,same_ids", EMBED_CASES)
def test_embedding_fwd_bwd(H, T_, with_tt, pos_beta, want_type, same_ids):
    """B = 9, S = 129: 1161 rows, 3 rows per block of the type-gradient kernel, rows % 4 = 1.
    H / 8 does not divide 256 at H = 768 and 1536: there the type gradient was counted twice in
    columns 0..511 before the kernel's idle threads were made to leave."""
    B, S, V = O.EMBED_B, O.EMBED_S, O.EMBED_V
    inp = _dev(O.embed_inputs(H, T_, same_ids, with_tt))
    s = Guarded((B * S, H), BF16)
    T.embed_fwd(inp["ids"], inp["tt"], inp["word"], inp["pos"], inp["typ"], S, out=s.t)
    want = O.embed_fwd(inp["ids"], inp["tt"], inp["word"], inp["pos"], inp["typ"], S)
    scale = O.embed_fwd(inp["ids"], inp["tt"], inp["word"].abs(), inp["pos"].abs(), inp["typ"].abs(), S)
    figs = {"emb_s": O.figure(s.t, want, scale, bf16_store=True)}
    dword = Guarded((V, H), F32, init=inp["dword0"])
    dpos = Guarded((S, H), F32, init=inp["dpos0"])
    dtyp = Guarded((T_, H), F32)
    T.embed_bwd(inp["ds"], inp["ids"], inp["tt"], dword.t, dpos.t, dtyp.t if want_type else None, B, S,
                pos_beta=pos_beta)
    torch.cuda.synchronize()
    a = (inp["ds"], inp["ids"], inp["tt"], inp["dword0"], inp["dpos0"], T_, B, S, pos_beta)
    rw, rp, rt = O.embed_bwd(*a)
    sw, sp, st = O.embed_bwd_abs(*a)
    figs["emb_dword"] = O.figure(dword.t, rw, sw)
    figs["emb_dpos"] = O.figure(dpos.t, rp, sp)
    if want_type:
        figs["emb_dtype"] = O.figure(dtyp.t, rt, st)
        if not with_tt:
            assert bool((dtyp.t[1:] == 0).all())
    else:
        assert bool((dtyp.raw == PATTERN).all())
    print("embedding", H, T_, with_tt, pos_beta, want_type, same_ids, {k: "%.2e" % v for k, v in figs.items()})
    O.check(figs, H)
    assert s.intact() and dword.intact() and dpos.intact() and dtyp.intact()
    named = torch.zeros(V, dtype=torch.bool, device=DEV)
    named[inp["ids"].long()] = True
    assert int((~named).sum()) >= 2 and _same_bits(dword.t[~named], inp["dword0"][~named])


def test_embedding_fwd_h4096_and_bwd_refuses_it():
    """The forward strides any H % 8 == 0; the type-gradient kernel holds a row's H / 8 chunks in one
    256-thread block, so the backward refuses H / 8 > 256."""
    B, S, H = O.EMBED_B, O.EMBED_S, 4096
    inp = _dev(O.embed_inputs(H, 2))
    s = Guarded((B * S, H), BF16)
    T.embed_fwd(inp["ids"], inp["tt"], inp["word"], inp["pos"], inp["typ"], S, out=s.t)
    want = O.embed_fwd(inp["ids"], inp["tt"], inp["word"], inp["pos"], inp["typ"], S)
    scale = O.embed_fwd(inp["ids"], inp["tt"], inp["word"].abs(), inp["pos"].abs(), inp["typ"].abs(), S)
    O.check({"emb_s": O.figure(s.t, want, scale, bf16_store=True)}, H)
    assert s.intact()
    dword, dpos, dtyp = Guarded((O.EMBED_V, H), F32), Guarded((S, H), F32), Guarded((2, H), F32)
    with pytest.raises(_lib.HipKernelError):
        T.embed_bwd(inp["ds"], inp["ids"], inp["tt"], dword.t, dpos.t, dtyp.t, B, S)
    torch.cuda.synchronize()
    assert all(bool((g.raw == PATTERN).all()) for g in (dword, dpos, dtyp))


# ------------------------------------------------------------------ gather / scatter
PAD = 8  # columns before a slice; the wide buffers have H + 3 * PAD columns


def _wide(rows, H, gen):
    """A Guarded [rows, H + 24] bf16 buffer of noise and its column slice [:, 8:8+H] (row stride > H)."""
    w = Guarded((rows, H + 3 * PAD), BF16, init=torch.randn(rows, H + 3 * PAD, generator=gen).to(BF16))
    return w, w.t[:, PAD:PAD + H]


def _gather_scatter(H, idx, group, n, R, gen):
    wide, src = _wide(R, H, gen)
    before = wide.t.clone()
    out = Guarded((n, H), BF16)
    T.gather_rows(src, idx, out=out.t, group=group, n=n)
    assert torch.equal(out.t, O.gather_rows(src, idx, group, n)) and out.intact()
    assert torch.equal(wide.t, before)
    # scatter other rows back into a slice of another wide buffer: the slice's named rows change,
    # nothing else does
    rows = torch.randn(n, H, generator=gen).to(BF16).to(DEV)
    for accumulate in (False, True):
        wd, dst = _wide(R, H, gen)
        expect = wd.t.clone().to(F64)
        abs_ = wd.t.clone().to(F64).abs()
        expect[:, PAD:PAD + H] = O.scatter_rows(rows, idx, dst, accumulate, group)
        abs_[:, PAD:PAD + H] = O.scatter_rows(rows.abs(), idx, dst.abs(), accumulate, group)
        T.scatter_rows(rows, idx, dst, accumulate=accumulate, group=group)
        torch.cuda.synchronize()
        assert wd.intact()
        if accumulate:
            figs = {"scatter": O.figure(wd.t, expect, abs_, bf16_store=True)}
            print("scatter", H, n, group, figs)
            O.check(figs, (H, n))
            to = O._targets(idx, n, group, DEV)
            mask = torch.ones_like(expect, dtype=torch.bool)
            mask[to, PAD:PAD + H] = False
            assert torch.equal(wd.t.to(F64)[mask], expect[mask])
        else:
            assert torch.equal(wd.t.to(F64), expect)


@pytest.mark.parametrize("H", O.GATHER_H)
@pytest.mark.parametrize("n", O.GATHER_N)
def test_gather_scatter_rows_strided_plain_index(H, n):
    gen = O._gen(H, n, 5)
    R = 40
    idx = torch.randperm(R, generator=gen)[:n].int().to(DEV)
    _gather_scatter(H, idx, (1, 0), n, R, gen)


@pytest.mark.parametrize("H", O.GATHER_H)
def test_gather_scatter_rows_strided_grouped_and_cls(H):
    """The engine's forms: positions [B, P] per sequence of a [B*S, H] activation, group = (P, S),
    and every sequence's first row, no index, group = (1, S)."""
    gen = O._gen(H, 6)
    B, S, P = 5, 8, 3
    pos = torch.stack([torch.randperm(S, generator=gen)[:P] for _ in range(B)]).int().to(DEV)
    _gather_scatter(H, pos.reshape(-1), (P, S), B * P, B * S, gen)
    _gather_scatter(H, None, (1, S), B, B * S, gen)


# ------------------------------------------------------------------ dact, tanh_
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n8", O.DACT_N8)
def test_dact(kind, n8):
    aux, dy = (t.to(DEV) for t in (O.act_inputs(n8 * 8) if kind == 0 else O.tanh_outputs(n8 * 8)))
    out = Guarded((n8 * 8,), BF16)
    T.dact(dy, aux, kind, out=out.t)
    figs = {"dact": O.figure(out.t, O.dact(dy, aux, kind), dy.to(F64).abs(), bf16_store=True)}
    print("dact", kind, n8, figs)
    O.check(figs, (kind, n8))
    assert out.intact()


@pytest.mark.parametrize("n", O.TANH_N)
def test_tanh_in_place(n):
    x, _ = O.act_inputs(n)
    buf = Guarded((n,), BF16, init=x)
    T.tanh_(buf.t)
    figs = {"tanh": O.figure(buf.t, O.tanh(x.to(DEV)), 1.0, bf16_store=True)}
    print("tanh", n, figs)
    O.check(figs, n)
    assert buf.intact()
