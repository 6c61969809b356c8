"""RMSNorm and SwiGLU: the kernels of rmsnorm_glu.hip behind `ops.transformer.rmsnorm_fwd / rmsnorm_bwd /
swiglu_fwd / swiglu_bwd` and `ops.kernels.rms_generic_*`, `ttd.nn.rms_norm / swiglu` (GPU kernels and
CPU paths), `layers.RMSNormalization / SwiGLU` and the BERT engine (`BertConfig.rms_norm`,
`BertConfig.gated_ffn`).

Definitions (all fp32):
  RMSNorm   s = res + drop_in(x);  rstd = rsqrt(mean_j(s_j^2) + eps);  y = drop_out(s * rstd * gamma)
            n = s * rstd, g = drop_out'(dy) * gamma:  ds = rstd * (g - n * mean_j(g_j n_j)),
            dx = ds * mask_in * scale_in,  dgamma = sum_rows drop_out'(dy) * n
  SwiGLU    x2 = [a | b]:  h = a * sigmoid(a) * b;  da = dh * b * sig * (1 + a * (1 - sig)),  db = dh * a * sig

Bars. The fast RMSNorm is held to the LayerNorm bars of test_kernels_transformer.py (s: atol 2e-2,
rtol 1e-2; y: atol 5e-2, rtol 2e-2; gradients: relative L2 < 2e-2). The generic RMSNorm and the fp32
SwiGLU use the measure of test_nn_gpu_ops.py, max |error| / max |reference| (fp32 1e-5 forward, 1e-4
backward; bf16 2e-2 / 3e-2), against a float64 oracle of the same inputs. For the generic dx the
denominator is not allowed to fall below max |rstd * dy * gamma|, the size of the terms the formula
subtracts: at width 1 the exact dx is dy * gamma * eps / |x|^3 (about 1e-6 of those terms), which no
fp32 evaluation of rstd * (dy * gamma - n * mean(dy * gamma * n)) resolves, the torch fp32 autograd
included; at the other widths the two denominators are of one size. The bf16 SwiGLU is held to the
GELU / dGELU bar (atol = rtol = 3e-2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tensorflow_train_distributed_amd as ttd
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.models.bert import BertConfig, BertPretraining, synthetic_batch
from tensorflow_train_distributed_amd.ops import kernels as K
from tensorflow_train_distributed_amd.ops import transformer as T
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ oracles (written here, not in the package)
def _rms_ref(x, gamma, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * gamma


def _rms_grads(x, gamma, dy, eps):
    """The closed-form backward of the issue, any float dtype."""
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    n = x * rstd
    g = dy * gamma
    dx = rstd * (g - n * (g * n).mean(-1, keepdim=True))
    return dx, (dy * n).reshape(-1, x.shape[-1]).sum(0)


def _swiglu_ref(x2):
    I = x2.shape[-1] // 2
    a, b = x2[..., :I], x2[..., I:]
    return a * torch.sigmoid(a) * b


def _swiglu_grads(x2, dh):
    I = x2.shape[-1] // 2
    a, b = x2[..., :I], x2[..., I:]
    sg = torch.sigmoid(a)
    return torch.cat([dh * b * sg * (1 + a * (1 - sg)), dh * a * sg], dim=-1)


def _err(got, want, floor=0.0):
    """max |got - want| / max(max |want|, floor): the measure of test_nn_gpu_ops.py."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / max(float(want.abs().max()), floor, 1e-30))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _oracle_backward_is_float64_autograd():
    """The closed-form backwards above against float64 autograd of the forward formulas."""
    torch.manual_seed(2)
    x = torch.randn(6, 10, dtype=torch.float64, requires_grad=True)
    gamma = torch.randn(10, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(6, 10, dtype=torch.float64)
    _rms_ref(x, gamma, 1e-6).backward(dy)
    dx, dg = _rms_grads(x.detach(), gamma.detach(), dy, 1e-6)
    torch.testing.assert_close(x.grad, dx, atol=1e-12, rtol=1e-10)
    torch.testing.assert_close(gamma.grad, dg, atol=1e-12, rtol=1e-10)
    x2 = (torch.randn(6, 10, dtype=torch.float64) * 4).requires_grad_(True)
    dh = torch.randn(6, 5, dtype=torch.float64)
    _swiglu_ref(x2).backward(dh)
    torch.testing.assert_close(x2.grad, _swiglu_grads(x2.detach(), dh), atol=1e-12, rtol=1e-10)


# ------------------------------------------------------------------ CPU: ttd.nn
def test_nn_rms_norm_cpu_is_the_formula():
    _oracle_backward_is_float64_autograd()
    torch.manual_seed(0)
    x = torch.randn(3, 5, 24, requires_grad=True)
    gamma = (torch.randn(24) * 0.5 + 1).requires_grad_(True)
    y = N.rms_norm(x, gamma, 1e-5)
    assert y.shape == x.shape and y.dtype == torch.float32
    torch.testing.assert_close(y, _rms_ref(x.detach(), gamma.detach(), 1e-5), atol=1e-6, rtol=1e-5)
    assert not torch.allclose(y, F.layer_norm(x, (24,), gamma, None, 1e-5), atol=1e-2)  # no centring
    dy = torch.randn(3, 5, 24)
    y.backward(dy)
    dx, dg = _rms_grads(x.detach().double(), gamma.detach().double(), dy.double(), 1e-5)
    torch.testing.assert_close(x.grad.double(), dx, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(gamma.grad.double(), dg, atol=1e-5, rtol=1e-4)
    # default eps is 1e-6
    torch.testing.assert_close(N.rms_norm(x.detach(), gamma.detach()), _rms_ref(x.detach(), gamma.detach(), 1e-6),
                               atol=1e-6, rtol=1e-5)


def test_nn_swiglu_cpu_is_the_formula():
    _oracle_backward_is_float64_autograd()
    torch.manual_seed(1)
    x = (torch.randn(4, 7, 26) * 3).requires_grad_(True)
    h = N.swiglu(x)
    assert h.shape == (4, 7, 13)
    torch.testing.assert_close(h, _swiglu_ref(x.detach()), atol=1e-6, rtol=1e-5)
    torch.testing.assert_close(h, F.silu(x.detach()[..., :13]) * x.detach()[..., 13:], atol=1e-6, rtol=1e-5)
    dh = torch.randn(4, 7, 13)
    h.backward(dh)
    torch.testing.assert_close(x.grad.double(), _swiglu_grads(x.detach().double(), dh.double()), atol=1e-5, rtol=1e-4)


def test_nn_rms_norm_and_swiglu_refusals_cpu():
    with pytest.raises(InvalidArgumentError):
        N.swiglu(torch.randn(3, 7))                    # odd last dimension
    with pytest.raises(InvalidArgumentError):
        N.swiglu(torch.randn(3, 0))
    with pytest.raises(InvalidArgumentError):
        N.rms_norm(torch.randn(3, 8), torch.ones(7))   # gamma of another width
    with pytest.raises(InvalidArgumentError):
        N.rms_norm(torch.randn(3, 8), torch.ones(1, 8))


# ------------------------------------------------------------------ CPU: layers
def test_layers_variables():
    L.reset_naming(0)
    x = torch.randn(2, 5, 12)
    rms, glu, glu_nb = L.RMSNormalization(), L.SwiGLU(20), L.SwiGLU(6, use_bias=False)
    with torch.no_grad():
        y, h, h2 = rms(x), glu(x), glu_nb(x)
    assert rms.epsilon == 1e-6 and L.RMSNormalization(epsilon=1e-5).epsilon == 1e-5
    assert [(n, tuple(t.shape)) for n, t in rms.named_variables()] == [("rms_normalization/gamma", (12,))]
    assert torch.equal(rms.gamma.detach(), torch.ones(12))
    assert [(n, tuple(t.shape)) for n, t in glu.named_variables()] == [("swiglu/kernel", (12, 40)),
                                                                        ("swiglu/bias", (40,))]
    assert [(n, tuple(t.shape)) for n, t in glu_nb.named_variables()] == [("swiglu_1/kernel", (12, 12))]
    assert y.shape == x.shape and h.shape == (2, 5, 20) and h2.shape == (2, 5, 6)
    torch.testing.assert_close(y, _rms_ref(x, torch.ones(12), 1e-6), atol=1e-6, rtol=1e-5)
    # gate columns first: call = swiglu(dense(x))
    z = x @ glu.kernel.detach() + glu.bias.detach()
    torch.testing.assert_close(h, F.silu(z[..., :20]) * z[..., 20:], atol=1e-5, rtol=1e-4)


def test_sequential_with_rmsnorm_and_swiglu_trains_under_gradient_tape():
    L.reset_naming(seed=5)
    torch.manual_seed(3)
    model = L.Sequential([L.Dense(16), L.RMSNormalization(), L.SwiGLU(24), L.Dense(4)])
    X, Y = torch.randn(32, 8), torch.randint(0, 4, (32,))
    model(X[:1])
    flat = model.to_flat("cpu")
    assert len(flat.names()) == 7  # 2 + 1 + 2 + 2
    opt = ttd.train.MomentumOptimizer(0.1, 0.9)
    before = flat.master.clone()
    losses = []
    for _ in range(8):
        with ttd.GradientTape() as tape:
            loss = F.cross_entropy(model(X), Y)
        grads = tape.gradient(loss, model.trainable_variables)
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
        opt.apply_gradients(zip(grads, model.trainable_variables))
        losses.append(float(loss.detach()))
    assert not torch.equal(flat.master, before)
    assert losses[-1] < losses[0], losses


# ------------------------------------------------------------------ CPU: BERT configuration
def _tiny_cfg(**kw):
    return BertConfig(vocab_size=1000, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                      intermediate_size=256, max_position_embeddings=128, **kw)


def test_bert_config_flags_default_off_and_change_only_the_ffn1_shapes():
    assert BertConfig().rms_norm is False and BertConfig().gated_ffn is False
    base = {s.name: s for s in BertPretraining.build_specs(_tiny_cfg())}
    order = [s.name for s in BertPretraining.build_specs(_tiny_cfg())]
    Lc, Hc, Ic = 2, 128, 256
    for flags in (dict(rms_norm=True), dict(gated_ffn=True), dict(rms_norm=True, gated_ffn=True)):
        specs = BertPretraining.build_specs(_tiny_cfg(**flags))
        assert [s.name for s in specs] == order, flags
        changed = sorted(s.name for s in specs if tuple(s.shape) != tuple(base[s.name].shape))
        if flags.get("gated_ffn"):
            want = sorted("bert/encoder/layer_%d/intermediate/dense/%s" % (l, k) for l in range(Lc)
                          for k in ("kernel", "bias"))
            assert changed == want
            by = {s.name: s for s in specs}
            k0 = by["bert/encoder/layer_0/intermediate/dense/kernel"]
            assert tuple(k0.shape) == (2 * Ic, Hc) and k0.meta["tf_shape"] == (Hc, 2 * Ic)
            assert tuple(by["bert/encoder/layer_0/intermediate/dense/bias"].shape) == (2 * Ic,)
            assert tuple(by["bert/encoder/layer_0/output/dense/kernel"].shape) == (Hc, Ic)
            grow = Lc * (Ic * Hc + Ic)
        else:
            assert changed == []
            grow = 0
        assert (BertPretraining.count_parameters(_tiny_cfg(**flags))
                == BertPretraining.count_parameters(_tiny_cfg()) + grow)
    big = BertPretraining.count_parameters(BertConfig.large(gated_ffn=True))
    assert big == 336226108 + 24 * (4096 * 1024 + 4096)


def test_bert_gated_checkpoint_round_trips_in_tf_layout(tmp_path):
    from tensorflow_train_distributed_amd.train import checkpoint as C
    cfg = BertConfig(vocab_size=1000, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                     intermediate_size=256, max_position_embeddings=128, gated_ffn=True, rms_norm=True)
    m = BertPretraining(cfg, device="cpu", seed=1)
    path = C.Saver(m.params).save(None, str(tmp_path / "model.ckpt"), global_step=3)
    shapes = dict(C.list_variables(path))
    assert shapes["bert/encoder/layer_0/intermediate/dense/kernel"] == (128, 512)
    assert shapes["bert/encoder/layer_0/intermediate/dense/bias"] == (512,)
    assert shapes["bert/encoder/layer_0/output/dense/kernel"] == (256, 128)
    assert shapes["bert/encoder/layer_0/output/LayerNorm/beta"] == (128,)
    k = C.load_variable(path, "bert/encoder/layer_0/intermediate/dense/kernel")
    torch.testing.assert_close(torch.from_numpy(k), m.params.var["bert/encoder/layer_0/intermediate/dense/kernel"].t())
    m2 = BertPretraining(cfg, device="cpu", seed=2)
    assert not torch.equal(m2.params.master, m.params.master)
    C.Saver(m2.params).restore(None, path)
    assert torch.equal(m2.params.master, m.params.master)


def test_bert_reference_loss_flags_cpu():
    torch.manual_seed(0)
    batch = synthetic_batch(_tiny_cfg(), 2, 32, max_predictions=4, device="cpu", seed=1)

    def run(**flags):
        m = BertPretraining(_tiny_cfg(**flags), device="cpu", seed=3, dropout=False)
        g = torch.Generator().manual_seed(9)
        leaves = {}
        for n in m.params.names():
            t = m.params.var[n].detach().clone()
            if "LayerNorm" in n:  # away from (1, 0), so that a read of beta would show
                t += torch.randn(t.shape, generator=g) * 0.1
            leaves[n] = t.requires_grad_(True)
        mlm, nsp = m.reference_loss(batch, leaves)
        (mlm + nsp).backward()
        return float(mlm.detach()), leaves

    plain, lp = run()
    rms, lr = run(rms_norm=True)
    gated, lg = run(gated_ffn=True)
    both, lb = run(rms_norm=True, gated_ffn=True)
    print("mlm loss: plain %.6f, rms_norm %.6f, gated_ffn %.6f, both %.6f" % (plain, rms, gated, both))
    assert len({plain, rms, gated, both}) == 4
    for v in (plain, rms, gated, both):
        assert v == v and 0 < v < 20
    betas = [n for n in lp if n.endswith("LayerNorm/beta")]
    assert len(betas) == 2 * 2 + 2
    for n in betas:
        assert lp[n].grad is not None and float(lp[n].grad.abs().sum()) > 0
        assert lg[n].grad is not None
        assert lr[n].grad is None and lb[n].grad is None, n
    for n in lp:
        if n not in betas:
            assert lr[n].grad is not None and lb[n].grad is not None, n
    k = "bert/encoder/layer_0/intermediate/dense/kernel"
    assert tuple(lg[k].grad.shape) == (512, 128) and tuple(lp[k].grad.shape) == (256, 128)


# ------------------------------------------------------------------ GPU: RMSNorm, fast widths
@gpu
@pytest.mark.parametrize("H,rows", [(512, 300), (1024, 300), (1024, 5003), (512, 4099), (1536, 300), (2048, 77),
                                    (4096, 300), (1024, 1), (512, 3)])
def test_rmsnorm_residual_dropout_fwd_bwd(H, rows):
    # the shapes of test_layernorm_residual_dropout_fwd_bwd (rows >= 4096: many rows per block, odd
    # tails; each H its own kernel variant) plus 1 and 3 rows: a partly filled 4-row forward block
    torch.manual_seed(1)
    dev = "cuda"
    x = torch.randn(rows, H, device=dev).bfloat16()
    res = torch.randn(rows, H, device=dev).bfloat16()
    gamma = torch.randn(H, device=dev) * 0.5 + 1
    p_in, p_out, eps = 0.1, 0.2, 1e-6
    rng = T.RngState(7, dev)
    y, s, rstd = T.rmsnorm_fwd(x, gamma, res=res, eps=eps, p_in=p_in, site_in=11, p_out=p_out, site_out=12, rng=rng)
    seed, step = rng.host()
    idx = np.arange(rows * H, dtype=np.int64)
    kin = torch.from_numpy(T.keep_mask(seed, step, 11, p_in, idx).reshape(rows, H)).float().to(dev)
    kout = torch.from_numpy(T.keep_mask(seed, step, 12, p_out, idx).reshape(rows, H)).float().to(dev)
    xf = x.float().requires_grad_(True)
    rf = res.float().requires_grad_(True)
    gf = gamma.clone().requires_grad_(True)
    sref = rf + xf * kin / (1 - p_in)
    yref = _rms_ref(sref, gf, eps) * kout / (1 - p_out)
    assert s.shape == (rows, H) and s.dtype == torch.bfloat16 and rstd.shape == (rows,)
    torch.testing.assert_close(s.float(), sref.detach(), atol=2e-2, rtol=1e-2)
    torch.testing.assert_close(y.float(), yref.detach(), atol=5e-2, rtol=2e-2)
    torch.testing.assert_close(rstd, torch.rsqrt(s.float().pow(2).mean(-1) + eps), atol=1e-6, rtol=1e-5)
    dy = torch.randn(rows, H, device=dev).bfloat16()
    yref.backward(dy.float())
    dg = torch.empty(H, device=dev)
    ds, dx = T.rmsnorm_bwd(dy, s, rstd, gamma, dg, want_dx=True, p_in=p_in, site_in=11, p_out=p_out, site_out=12,
                           rng=rng)
    rels = {name: _rel(got.float(), want) for name, got, want in
            (("dres", ds, rf.grad), ("dx", dx, xf.grad), ("dgamma", dg, gf.grad))}
    print("H %d rows %d: relative L2 %s" % (H, rows, rels))
    for name, rel in rels.items():
        assert rel < 2e-2, (name, rel)


@gpu
def test_rmsnorm_plain_accumulate_and_reproducible():
    torch.manual_seed(2)
    dev, rows, H = "cuda", 4099, 1024
    x = torch.randn(rows, H, device=dev).bfloat16()
    gamma = torch.randn(H, device=dev) * 0.5 + 1
    y, s, rstd = T.rmsnorm_fwd(x, gamma)
    assert s is x                      # no residual, no input dropout: nothing to save
    torch.testing.assert_close(y.float(), _rms_ref(x.float(), gamma, 1e-6), atol=5e-2, rtol=2e-2)
    dy = torch.randn(rows, H, device=dev).bfloat16()
    work = T.rmsnorm_bwd_workspace(rows, H, dev)
    assert work.dtype == torch.float32 and work.shape[1] == H
    dg1, dg2 = torch.empty(H, device=dev), torch.full((H,), float("nan"), device=dev)
    ds1, none = T.rmsnorm_bwd(dy, s, rstd, gamma, dg1, work=work)
    assert none is None
    ds2, _ = T.rmsnorm_bwd(dy, s, rstd, gamma, dg2)
    assert torch.equal(_bits(dg1), _bits(dg2))           # fixed summation order: bit for bit
    assert torch.equal(_bits(ds1), _bits(ds2))
    dxw, dgw = _rms_grads(x.double(), gamma.double(), dy.double(), 1e-6)
    assert _rel(ds1, dxw) < 2e-2 and _rel(dg1, dgw) < 2e-2
    acc = torch.full((H,), 2.0, device=dev)
    T.rmsnorm_bwd(dy, s, rstd, gamma, acc, accumulate=True, work=work)
    torch.testing.assert_close(acc, dg1 + 2.0, atol=1e-5, rtol=1e-6)
    T.rmsnorm_bwd(dy, s, rstd, gamma, acc, accumulate=False, work=work)
    assert torch.equal(_bits(acc), _bits(dg1))


# ------------------------------------------------------------------ GPU: RMSNorm, any width
@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [1, 7, 64, 100, 1000, 5000])
def test_rmsnorm_generic_any_width(H, dtype):
    torch.manual_seed(3)
    rows, eps = 9, 1e-6
    x = torch.randn(rows, H).to(dtype)
    dy = torch.randn(rows, H).to(dtype)
    gamma = torch.randn(H) * 0.5 + 1
    want = _rms_ref(x.double(), gamma.double(), eps)
    dxw, dgw = _rms_grads(x.double(), gamma.double(), dy.double(), eps)
    y, rstd = K.rms_generic_fwd(x.cuda(), gamma.cuda(), eps)
    assert y.dtype == dtype and y.shape == (rows, H)
    dg = torch.full((H,), float("nan"), device="cuda")
    dx = K.rms_generic_bwd(dy.cuda(), x.cuda(), gamma.cuda(), rstd, dg)
    dg2 = torch.empty(H, device="cuda")
    assert K.rms_generic_bwd(dy.cuda(), x.cuda(), gamma.cuda(), rstd, dg2, want_dx=False) is None
    assert torch.equal(_bits(dg), _bits(dg2))
    rs = torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + eps)
    terms = float((rs * dy.double() * gamma.double()).abs().max())
    e = dict(y=_err(y, want), rstd=_err(rstd, rs.flatten()), dx=_err(dx, dxw, floor=terms), dgamma=_err(dg, dgw))
    print("H %d %s: max error / max reference %s" % (H, dtype, e))
    fwd, bwd = (1e-5, 1e-4) if dtype == torch.float32 else (2e-2, 3e-2)
    assert e["y"] <= fwd and e["rstd"] <= 1e-5, e
    assert e["dx"] <= bwd and e["dgamma"] <= bwd, e


# ------------------------------------------------------------------ GPU: SwiGLU
def _glu_inputs(rows, I, dtype, padded, seed):
    """x2 [rows, 2I], dh [rows, I] (and sentinel-filled outputs) on the GPU, dense or as column views
    of wider buffers; |gate| reaches 30."""
    g = torch.Generator().manual_seed(seed)
    pad = 24 if padded else 0

    def view(t, fill=None):
        buf = torch.full((rows, t.shape[1] + pad), -77.0).to(dtype)
        buf[:, :t.shape[1]] = t
        buf = buf.cuda()
        return buf, buf[:, :t.shape[1]] if pad else buf

    x2 = torch.randn(rows, 2 * I, generator=g) * 3
    x2.view(-1)[::5] = torch.linspace(-30, 30, x2.view(-1)[::5].numel())
    dh = torch.randn(rows, I, generator=g)
    _, xv = view(x2.to(dtype).float())
    _, dv = view(dh.to(dtype).float())
    hbuf, hv = view(torch.zeros(rows, I) - 77.0)
    obuf, ov = view(torch.zeros(rows, 2 * I) - 77.0)
    return xv, dv, hbuf, hv, obuf, ov


def _check_glu(rows, I, dtype, padded):
    xv, dv, hbuf, hv, obuf, ov = _glu_inputs(rows, I, dtype, padded, seed=rows + I)
    x64, d64 = xv.double().cpu(), dv.double().cpu()
    assert float(x64[:, :I].abs().max()) >= 29.0 or rows * I < 3
    before = xv.clone()
    h = T.swiglu_fwd(xv, out=hv)
    dx2 = T.swiglu_bwd(dv, xv, out=ov)
    assert h.data_ptr() == hv.data_ptr() and dx2.data_ptr() == ov.data_ptr()
    if padded:  # the pad columns are not written
        assert bool((hbuf[:, I:].float() == -77.0).all()) and bool((obuf[:, 2 * I:].float() == -77.0).all())
    assert torch.equal(_bits(xv), _bits(before))
    hw, dw = _swiglu_ref(x64), _swiglu_grads(x64, d64)
    assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(dx2.float()).all())
    if dtype == torch.bfloat16:
        torch.testing.assert_close(h.double().cpu(), hw, atol=3e-2, rtol=3e-2)
        torch.testing.assert_close(dx2.double().cpu(), dw, atol=3e-2, rtol=3e-2)
    else:
        e = (_err(h, hw), _err(dx2, dw))
        print("rows %d I %d fp32%s: max error / max reference fwd %.3g bwd %.3g"
              % (rows, I, " padded" if padded else "", *e))
        assert e[0] <= 1e-5 and e[1] <= 1e-4, e
    # without out=: fresh dense results, the same bits
    assert torch.equal(_bits(T.swiglu_fwd(xv)), _bits(h))
    assert torch.equal(_bits(T.swiglu_bwd(dv, xv)), _bits(dx2))
    # in place over the forward's input
    inplace = T.swiglu_bwd(dv, xv, out=xv)
    assert inplace.data_ptr() == xv.data_ptr()
    assert torch.equal(_bits(xv), _bits(dx2))


@gpu
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows", [1, 3, 300])
@pytest.mark.parametrize("I", [1, 8, 100, 1024])
def test_swiglu_kernel_matches_oracle(I, rows, dtype, padded):
    _check_glu(rows, I, dtype, padded)


@gpu
def test_swiglu_kernel_grid_stride_coverage():
    """More work items (rows * I / 8 for bf16) than the capped grid has threads."""
    rows, I = 4100, 1536
    assert rows * I // 8 > T.swiglu_max_threads()
    _check_glu(rows, I, torch.bfloat16, True)


@gpu
def test_swiglu_extreme_gates_do_not_overflow():
    """exp(-a) overflows fp32 below a = -88: the unit and its gradient must come out 0, not NaN."""
    a = torch.tensor([-200.0, -100.0, -89.0, -30.0, 0.0, 30.0, 89.0, 200.0])
    for dtype in (torch.float32, torch.bfloat16):
        x2 = torch.cat([a, torch.full((8,), 1.5)]).to(dtype).reshape(1, 16).cuda()
        dh = torch.ones(1, 8, dtype=dtype, device="cuda")
        h, dx2 = T.swiglu_fwd(x2), T.swiglu_bwd(dh, x2)
        assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(dx2.float()).all())
        x64 = x2.double().cpu()
        torch.testing.assert_close(h.double().cpu(), _swiglu_ref(x64), atol=1e-5, rtol=3e-2)
        torch.testing.assert_close(dx2.double().cpu(), _swiglu_grads(x64, dh.double().cpu()), atol=1e-5, rtol=3e-2)
        assert float(h[0, 0]) == 0.0 and float(dx2[0, 0]) == 0.0 and float(dx2[0, 8]) == 0.0


# ------------------------------------------------------------------ GPU: refusals
@gpu
def test_rmsnorm_and_swiglu_refusals():
    dev = "cuda"
    x = torch.randn(8, 1024, device=dev).bfloat16()
    gamma = torch.ones(1024, device=dev)
    y, s, rstd = T.rmsnorm_fwd(x, gamma)
    dy, dg = torch.randn_like(x), torch.empty(1024, device=dev)
    with pytest.raises(InvalidArgumentError):      # fp16
        T.rmsnorm_fwd(x.half(), gamma)
    with pytest.raises(InvalidArgumentError):      # fp32 activations on the fast path
        T.rmsnorm_fwd(x.float(), gamma)
    with pytest.raises(InvalidArgumentError):      # not a fast width
        T.rmsnorm_fwd(torch.randn(8, 768, device=dev).bfloat16(), torch.ones(768, device=dev))
    off = torch.zeros(8 * 1024 + 4, device=dev, dtype=torch.bfloat16)[4:].view(8, 1024)
    assert off.is_contiguous() and off.data_ptr() % 16 == 8
    with pytest.raises(InvalidArgumentError):      # 16-byte loads from an 8-byte-aligned view
        T.rmsnorm_fwd(off, gamma)
    with pytest.raises(InvalidArgumentError):
        T.rmsnorm_fwd(x, gamma, out=off)
    with pytest.raises(InvalidArgumentError):      # a column view: rows are not dense
        T.rmsnorm_fwd(torch.zeros(8, 2048, device=dev, dtype=torch.bfloat16)[:, :1024], gamma)
    with pytest.raises(InvalidArgumentError):
        T.rmsnorm_fwd(x, gamma[:512])
    with pytest.raises(InvalidArgumentError):      # dropout without a generator state
        T.rmsnorm_fwd(x, gamma, p_out=0.1)
    with pytest.raises(InvalidArgumentError):      # workspace of the wrong size
        T.rmsnorm_bwd(dy, s, rstd, gamma, dg, work=torch.empty(3, device=dev))
    with pytest.raises(InvalidArgumentError):
        T.rmsnorm_bwd(dy, s, rstd, gamma, dg, work=torch.empty((4, 1024), device=dev, dtype=torch.bfloat16))
    with pytest.raises(InvalidArgumentError):
        T.rmsnorm_bwd(off, s, rstd, gamma, dg)
    with pytest.raises(InvalidArgumentError):
        T.rmsnorm_bwd(dy, s, rstd, gamma, dg[:512])
    x2 = torch.randn(8, 64, device=dev)
    with pytest.raises(InvalidArgumentError):      # odd 2I
        T.swiglu_fwd(x2[:, :63])
    with pytest.raises(InvalidArgumentError):
        T.swiglu_fwd(x2.half())
    with pytest.raises(InvalidArgumentError):      # column stride 2
        T.swiglu_fwd(x2[:, ::2])
    with pytest.raises(InvalidArgumentError):
        T.swiglu_fwd(x2.t())
    with pytest.raises(InvalidArgumentError):      # out of another width / dtype
        T.swiglu_fwd(x2, out=torch.empty(8, 16, device=dev))
    with pytest.raises(InvalidArgumentError):
        T.swiglu_fwd(x2, out=torch.empty(8, 32, device=dev, dtype=torch.bfloat16))
    with pytest.raises(InvalidArgumentError):      # dh of another dtype / shape
        T.swiglu_bwd(torch.ones(8, 32, device=dev, dtype=torch.bfloat16), x2)
    with pytest.raises(InvalidArgumentError):
        T.swiglu_bwd(torch.ones(8, 16, device=dev), x2)
    with pytest.raises(InvalidArgumentError):
        T.swiglu_bwd(torch.ones(7, 32, device=dev), x2)
    # the ttd.nn surface
    with pytest.raises(InvalidArgumentError):
        N.rms_norm(torch.randn(4, 8, device=dev, dtype=torch.float16), torch.ones(8, device=dev))
    with pytest.raises(InvalidArgumentError):
        N.swiglu(torch.randn(4, 8, device=dev, dtype=torch.float16))
    with pytest.raises(InvalidArgumentError):
        N.swiglu(torch.randn(4, 7, device=dev))
    torch.cuda.synchronize()
    # an 8-byte-aligned SwiGLU view is not refused: it takes the scalar kernel
    v = torch.randn(8 * 64 + 2, device=dev)[2:].view(8, 64)
    torch.testing.assert_close(T.swiglu_fwd(v).double().cpu(), _swiglu_ref(v.double().cpu()), atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------ GPU: hipGraph
@gpu
def test_rmsnorm_and_swiglu_in_one_hip_graph():
    torch.manual_seed(7)
    dev, rows, H, I = "cuda", 300, 1024, 520
    rng = T.RngState(11, dev)
    gamma = torch.randn(H, device=dev) * 0.5 + 1
    x, res, dy = [torch.randn(rows, H, device=dev).bfloat16() for _ in range(3)]
    x2buf = torch.randn(rows, 2 * I + 8, device=dev).bfloat16()
    x2, dh = x2buf[:, :2 * I], torch.randn(rows, I, device=dev).bfloat16()
    work = T.rmsnorm_bwd_workspace(rows, H, dev)

    def outs():
        return dict(y=torch.empty_like(x), s=torch.empty_like(x), rstd=torch.empty(rows, device=dev),
                    ds=torch.empty_like(x), dx=torch.empty_like(x), dg=torch.empty(H, device=dev),
                    h=torch.empty(rows, I, device=dev, dtype=torch.bfloat16),
                    dx2=torch.empty(rows, 2 * I, device=dev, dtype=torch.bfloat16))

    def run(o):
        T.rmsnorm_fwd(x, gamma, res=res, p_in=0.1, site_in=3, p_out=0.1, site_out=4, rng=rng, out=o["y"],
                      s_out=o["s"], rstd=o["rstd"])
        T.rmsnorm_bwd(dy, o["s"], o["rstd"], gamma, o["dg"], ds_out=o["ds"], want_dx=True, dx_out=o["dx"], p_in=0.1,
                      site_in=3, p_out=0.1, site_out=4, rng=rng, work=work)
        T.swiglu_fwd(x2, out=o["h"])
        T.swiglu_bwd(dh, x2, out=o["dx2"])

    cap = outs()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run(cap)  # warm
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            run(cap)
    torch.cuda.current_stream().wait_stream(st)
    for _ in range(2):
        for t in (x, res, dy, x2buf, dh):
            t.copy_(torch.randn(t.shape, device=dev).bfloat16())
        for t in cap.values():
            t.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        eager = outs()
        run(eager)
        torch.cuda.synchronize()
        for n in cap:
            assert torch.equal(_bits(cap[n]), _bits(eager[n])), n
        assert float(cap["y"].float().abs().max()) > 1 and float(cap["dx2"].float().abs().max()) > 0.1


# ------------------------------------------------------------------ GPU: ttd.nn and ttd.layers
@gpu
@pytest.mark.parametrize("H,dtype", [(100, torch.float32), (768, torch.bfloat16), (1024, torch.float32),
                                     (1024, torch.bfloat16), (512, torch.bfloat16)])
def test_nn_rms_norm_gpu_matches_cpu_path(H, dtype):
    g = torch.Generator().manual_seed(15)
    x = torch.randn(3, 3, H, generator=g).to(dtype)
    gamma = torch.randn(H, generator=g) * 0.5 + 1
    dy = torch.randn(3, 3, H, generator=g)
    xc, gc = x.float().clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    xg, gg = x.clone().cuda().requires_grad_(True), gamma.clone().cuda().requires_grad_(True)
    yc, yg = N.rms_norm(xc, gc, 1e-5), N.rms_norm(xg, gg, 1e-5)
    assert yg.dtype == dtype and yg.shape == x.shape and yg.is_cuda
    fwd, bwd = (1e-5, 1e-4) if dtype == torch.float32 else (2e-2, 3e-2)
    yc.backward(dy)
    yg.backward(dy.to(dtype).cuda())
    assert xg.grad.dtype == dtype and gg.grad.dtype == torch.float32
    e = (_err(yg, yc), _err(xg.grad, xc.grad), _err(gg.grad, gc.grad))
    print("H %d %s: max error / max reference y %.3g dx %.3g dgamma %.3g" % (H, dtype, *e))
    assert e[0] <= fwd and e[1] <= bwd and e[2] <= bwd, e


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nn_swiglu_gpu_matches_cpu_path(dtype):
    g = torch.Generator().manual_seed(16)
    x = (torch.randn(3, 5, 200, generator=g) * 2).to(dtype)
    dh = torch.randn(3, 5, 100, generator=g)
    xc, xg = x.float().clone().requires_grad_(True), x.clone().cuda().requires_grad_(True)
    hc, hg = N.swiglu(xc), N.swiglu(xg)
    assert hg.dtype == dtype and hg.shape == (3, 5, 100) and hg.is_cuda
    hc.backward(dh)
    hg.backward(dh.to(dtype).cuda())
    if dtype == torch.float32:
        assert _err(hg, hc) <= 1e-5 and _err(xg.grad, xc.grad) <= 1e-4
    else:
        torch.testing.assert_close(hg.float().cpu(), hc.detach(), atol=3e-2, rtol=3e-2)
        torch.testing.assert_close(xg.grad.float().cpu(), xc.grad, atol=3e-2, rtol=3e-2)
    # a column slice of a wider projection: the op makes it dense itself
    wide = torch.randn(3, 5, 264, generator=g)
    torch.testing.assert_close(N.swiglu(wide.cuda()[..., :200]).cpu(), N.swiglu(wide[..., :200]), atol=1e-5, rtol=1e-5)


@gpu
def test_layers_rmsnorm_and_swiglu_gpu_match_cpu():
    L.reset_naming(0)
    torch.manual_seed(17)
    x = torch.randn(4, 6, 48)
    dy = torch.randn(4, 6, 20)

    def build():
        return L.Sequential([L.RMSNormalization(epsilon=1e-5), L.SwiGLU(20)])

    cpu, dev = build(), build()
    with torch.no_grad():
        cpu(x)
        for _, t in cpu.named_variables():
            t.add_(torch.randn(t.shape) * 0.2)
        dev(x.cuda())
        dev.load_state_dict(cpu.state_dict())

    def run(model, d):
        xi = x.clone().to(d).requires_grad_(True)
        y = model(xi)
        y.backward(dy.to(d))
        grads = {"x": xi.grad.cpu()}
        for n, t in model.named_variables():
            grads[n.split("/", 1)[1]] = t.grad.cpu()
        return y.detach().cpu(), grads

    want, gw = run(cpu, "cpu")
    got, gg = run(dev, "cuda")
    assert sorted(gg) == sorted(gw) and len(gg) == 4
    assert _err(got, want) <= 1e-5, _err(got, want)          # fp32 in, fp32 kernels throughout
    for n in gw:
        assert _err(gg[n], gw[n]) <= 1e-4, (n, _err(gg[n], gw[n]))


# ------------------------------------------------------------------ GPU: BERT engine
def _small_cfg(**kw):
    return BertConfig(vocab_size=1000, hidden_size=512, num_hidden_layers=2, num_attention_heads=8,
                      intermediate_size=1024, max_position_embeddings=256, **kw)


_BETA = "LayerNorm/beta"


@gpu
@pytest.mark.parametrize("flags", [dict(rms_norm=True), dict(gated_ffn=True),
                                   dict(rms_norm=True, gated_ffn=True, causal=True, rotary=True)],
                         ids=["rms_norm", "gated_ffn", "all"])
def test_bert_engine_flags_match_reference(flags):
    """The body and bars of test_rope.py's test_bert_engine_rotary_matches_reference. Without rotary
    the exact key/bias gradient is zero (softmax does not see q.b_k) and the engine's is bf16 rounding
    noise: it is then held, as in test_bert.py, to 5 % of the query/bias gradient; with rotary it is
    compared like every other tensor. Under rms_norm the beta gradient slots are filled with 3.0
    before the step and must read exactly 0.0 after it."""
    torch.manual_seed(0)
    cfg = _small_cfg(**flags)
    m = BertPretraining(cfg, device="cuda", seed=3, dropout=False)
    m.blaslt = 0
    batch = synthetic_batch(cfg, 2, 256, max_predictions=20, device="cuda", seed=1, full_length=False)
    P = m.params
    betas = [n for n in P.names() if n.endswith(_BETA)]
    assert len(betas) == 2 * 2 + 2
    for n in betas:
        P.g[n].fill_(3.0)
    sums = m.forward_backward(batch)
    torch.cuda.synchronize()
    leaves = {n: P.c[n].float().detach().clone().requires_grad_(True) for n in P.names()}
    for n in P.names():  # fp32 params used directly by the kernels (biases, LayerNorm)
        if n.endswith("/bias") or "LayerNorm" in n or n.endswith("output_bias"):
            leaves[n] = P.var[n].detach().clone().requires_grad_(True)
    mlm, nsp = m.reference_loss(batch, leaves)
    print("mlm %.5f (reference %.5f), nsp %.5f (reference %.5f)"
          % (float(sums[0]), float(mlm.detach()), float(sums[2]), float(nsp.detach())))
    mlm_ref, nsp_ref = float(mlm.detach()), float(nsp.detach())
    assert abs(float(sums[0]) - mlm_ref) < 0.02 * mlm_ref, (float(sums[0]), mlm_ref)
    assert abs(float(sums[2]) - nsp_ref) < 0.02 * nsp_ref + 1e-3, (float(sums[2]), nsp_ref)
    (mlm + nsp).backward()
    ge, gr = [], []
    bad = []
    for n in P.names():
        a = P.g[n].flatten()
        b = leaves[n].grad
        b = torch.zeros_like(a) if b is None else b.flatten()
        if "rows" in P.spec(n).meta:  # padded vocab rows: must be exactly zero
            rows = P.spec(n).meta["rows"]
            width = a.numel() // P.spec(n).shape[0]
            assert float(a[rows * width:].abs().sum()) == 0.0, n
        if cfg.rms_norm and n.endswith(_BETA):
            assert leaves[n].grad is None and float(a.abs().max()) == 0.0, (n, float(a.abs().max()))
        ge.append(a)
        gr.append(b)
        if n.endswith("key/bias") and not cfg.rotary:
            qn = float(P.g[n.replace("key/bias", "query/bias")].norm())
            print("%s: |engine| %.4g, |reference| %.4g, |query/bias grad| %.4g" % (n, float(a.norm()), float(b.norm()),
                                                                                 qn))
            assert float(a.norm()) < 0.05 * qn, (n, float(a.norm()), qn)
        elif b.norm() > 0:
            rel = float((a - b).norm() / b.norm())
            if n.endswith("key/bias"):
                print("%s: relative error %.4f, |a - b| %.4g, |b| %.4g" % (n, rel, float((a - b).norm()),
                                                                          float(b.norm())))
            if rel > 0.1:
                bad.append((n, rel))
    ge, gr = torch.cat(ge), torch.cat(gr)
    cos = float(torch.dot(ge, gr) / (ge.norm() * gr.norm()))
    print("gradient cosine %.5f" % cos)
    assert cos > 0.99, (cos, bad[:10])
    assert not bad, bad[:10]


@gpu
def test_bert_engine_norm_and_ffn_flags_are_live():
    """Dropout off: each flag changes the MLM loss on the same batch, and two runs with the flag on
    give the same loss bit for bit. One predicted position per sequence, for the reason given in
    test_rope.py's test_bert_engine_rotary_flag_is_live: the engine sums row losses with fp32 atomics
    and only a two-term sum is independent of their order."""
    torch.manual_seed(0)
    batch = synthetic_batch(_small_cfg(), 2, 256, max_predictions=1, device="cuda", seed=1)

    def losses(**flags):
        m = BertPretraining(_small_cfg(**flags), device="cuda", seed=3, dropout=False)
        m.blaslt = 0
        s = m.forward_backward(batch)
        torch.cuda.synchronize()
        return float(s[0]), float(s[2])

    plain = losses()
    for flags in (dict(rms_norm=True), dict(gated_ffn=True)):
        a, b = losses(**flags), losses(**flags)
        print("mlm / nsp loss: %s %r, again %r, plain %r" % (flags, a, b, plain))
        assert a == b, (flags, a, b)
        assert a[0] == a[0] and a[0] != plain[0], (flags, a, plain)


@gpu
def test_bert_training_with_both_flags_dropout_lamb_decreases_loss():
    """The body and bar of test_bert.py's test_bert_training_with_dropout_lamb_decreases_loss."""
    from tensorflow_train_distributed_amd.train.flat import FlatLAMB, Schedule
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=1000, hidden_size=512, num_hidden_layers=2, num_attention_heads=8,
                     intermediate_size=1024, max_position_embeddings=128, rms_norm=True, gated_ffn=True)
    m = BertPretraining(cfg, device="cuda", seed=4)
    opt = FlatLAMB(m.params, Schedule(kind=0, base_lr=2e-3), weight_decay=0.01)
    batch = synthetic_batch(cfg, 4, 128, max_predictions=20, device="cuda", seed=2)
    losses = []
    for _ in range(30):
        s = m.forward_backward(batch)
        opt.step()
        losses.append(float(s[0]))
    print("mlm loss: first %.4f, last %.4f" % (losses[0], losses[-1]))
    assert all(l == l for l in losses)
    assert losses[-1] < losses[0] - 1.0, losses
    for n in m.params.names():  # beta never moves: its gradient is zero every step
        if n.endswith(_BETA):
            assert float(m.params.var[n].abs().max()) == 0.0, n


@gpu
def test_bert_step_with_both_flags_segmented_capture_matches_eager():
    """The body and tolerances of test_bert.py's test_bert_step_segmented_capture_matches_eager."""
    from tensorflow_train_distributed_amd.train.flat import FlatLAMB, Schedule
    from tensorflow_train_distributed_amd.utils import graphs
    cfg = BertConfig(vocab_size=1000, hidden_size=512, num_hidden_layers=2, num_attention_heads=8,
                     intermediate_size=1024, max_position_embeddings=128, rms_norm=True, gated_ffn=True)
    batch = synthetic_batch(cfg, 4, 128, max_predictions=20, device="cuda", seed=2)

    def make():
        m = BertPretraining(cfg, device="cuda", seed=4, dropout=False)
        return m, FlatLAMB(m.params, Schedule(kind=0, base_lr=1e-3), weight_decay=0.01)

    m1, o1 = make()
    m2, o2 = make()
    assert m2.wgrad_stream

    def step(m, o):
        s = m.forward_backward(batch)
        o.step()
        return s

    eager = [step(m1, o1).clone() for _ in range(4)]
    main = torch.cuda.Stream(priority=torch.cuda.Stream.priority_range()[1])
    seg = graphs.capture_segmented(lambda: step(m2, o2), main=main, warmup=1)
    assert seg.info["streams"] == 2, seg.info
    replays = [seg.replay().clone() for _ in range(3)]
    torch.cuda.synchronize()
    for a, b in zip(eager[1:], replays):
        torch.testing.assert_close(a, b, rtol=3e-3, atol=3e-3)
    d = (m1.params.master - m2.params.master).abs().max()
    assert float(d) < 1e-3 * float(m1.params.master.abs().max()), float(d)
